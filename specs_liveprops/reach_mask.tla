------------------------------ MODULE reach_mask ------------------------------
(* Written to show: REACH RESPECTS THE MASK.  One fair process walks s = 0 -> 1 -> 2 <-> 3.  Q is s = 1.  The cycle {2, 3} is a fair component of the ~Q subgraph, but from the P state s = 0 it is reached through the Q state only: inside the mask s = 0 has no successor, its one-state component is unfair (the walker is enabled), and  (s = 0) ~> (s = 1)  HOLDS.  With the P state inside the ~Q region,  (s = 2) ~> (s = 1)  is VIOLATED. *)
EXTENDS Naturals

(* --algorithm reach_mask
variables s = 0;

fair process Walk = 0
begin
  W: while TRUE do
       either await s = 0; s := 1;
       or     await s = 1; s := 2;
       or     await s = 2; s := 3;
       or     await s = 3; s := 2;
       end either;
     end while;
end process

end algorithm *)

Through == (s = 0) ~> (s = 1)
Inside == (s = 2) ~> (s = 1)
=============================================================================
