------------------------------ MODULE ap_monotone_ok ------------------------------
(* ap_monotone without the branch down: Mono holds, and the search is the one without the PROPERTY. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_monotone_ok
variables x = 2;

process P \in 1..2
variable c = 0;
begin
  s: while c < 3 do
       x := x + 1;
       c := c + 1;
     end while;
end process

end algorithm *)

Mono == [][x' >= x]_x
=============================================================================
