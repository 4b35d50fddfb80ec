------------------------------ MODULE ap_always ------------------------------
(* [](x <= 3) as a PROPERTY is the INVARIANT x <= 3: same verdict, depth and behaviour. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_always
variables x = 0;

process P \in 1..2
begin
  s: while x < 5 do
       x := x + 1;
     end while;
end process

end algorithm *)

Small == [](x <= 3)
Le3 == x <= 3
=============================================================================
