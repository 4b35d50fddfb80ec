------------------------------ MODULE mask_split ------------------------------
(* Written to show: THE MASK SPLITS A COMPONENT.  One fair process counts modulo 3 for ever: the whole graph is one fair component, and every cycle passes the Q state c = 0.  The ~Q subgraph is the path c = 1 -> c = 2, acyclic; each of its states is a component of its own in which the fair process is enabled (at c = 2 by the edge that leaves the mask) and not taken, so none is fair and  []<>(c = 0)  HOLDS.  Components taken from the whole graph would call it violated. *)
EXTENDS Naturals

(* --algorithm mask_split
variables c = 0;

fair process Ring = 0
begin
  R: while TRUE do
       c := (c + 1) % 3;
     end while;
end process

end algorithm *)

Recurs == []<>(c = 0)
=============================================================================
